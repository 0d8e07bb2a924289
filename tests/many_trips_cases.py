"""The batches of tests/test_gpu_many_trips.py (on the device) and tests/test_many_trips_cases.py (the references alone, on the
CPU): work lists longer than a persistent launch can hold, made of the smallest items each kernel admits, so that every wave or
workgroup goes round its loop several times.  Every builder takes the device's CU count and returns the batch together with the
length of its work list BY THE DOCUMENTED RULE (a chunk, a record, a tile, a unit), which the tests assert before anything runs.

"What a launch can hold" is, for every case, the larger of today's cap at the launch site and what the CUs keep resident:
MAX_WAVES_PER_CU = 32 waves, hence floor(32 / waves per workgroup) workgroups.  The formulas are with the builders.

Shapes come from seeded generators, never from `k % m`: the grid's size is unknown here, and a short period could line up with
it.  Built once per (case, CU count) and kept, expected arenas included.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import dsd_pcm_cases as DC
import ohm_textbook as OT
import oracle_lib as O
import src_pull_model as PM
from device_shape import MAX_WAVES_PER_CU
from ohpipeline_amd import capi

FILL = 0xA5
LE, BE = O.ENDIAN_LITTLE, O.ENDIAN_BIG
kMax = O.RAMP_MAX
RAMPS = [(kMax, 0), (0, kMax), (kMax, 8192), (8191, 8190), (5, 5), (kMax, kMax), (0, 0), (12345, 54), (17, 16001)]
SAMPLE_EVERY = 61           # the pure-Python models check every 61st item (a prime: no period of a builder lines up with it)


# ---------------------------------------------------------------- the PCM line kernel (csrc/pcm_line_kernel.hip)
LINE_WAVES = 4              # kLineWaves: waves per workgroup
LINE_GROUPS_PER_CU = 6      # launch_line's cap today (6 workgroups per CU, 4 for large plain launches)
CHUNK_SUB = 512             # kChunkSub: subsamples per staged chunk
PLAIN, RAMPED, ATTENUATED, SILENT = "plain", "ramped", "attenuated", "silent"


def line_waves(cus):
    """The waves a line-kernel launch can hold: max(today's 6 x 4 per CU, the 32 a CU keeps resident) = 32 x CUs."""
    return max(LINE_GROUPS_PER_CU * LINE_WAVES, MAX_WAVES_PER_CU // LINE_WAVES * LINE_WAVES) * cus


def staged_need(cus):
    """Item 1: one chunk per wave and trip; more than three trips for every wave, and an odd remainder."""
    return 3 * line_waves(cus) + 131


def register_need(cus):
    """Item 2: two chunks per wave and trip; more than two trips for every wave, and an odd remainder."""
    return 2 * 2 * line_waves(cus) + 131


def stage_loads(src_offset, src_bytes):
    """How many loads stage_in issues for a chunk: 64 lanes x 16-byte pieces, from the aligned piece its first byte lies in (the
    arenas are 16-byte aligned on the device, so the offset's residue is the address's)."""
    pieces = (src_offset % 16 + src_bytes + 15) // 16
    return (pieces + 63) // 64


def _msg_fields(rng, kind):
    ramp = RAMPS[int(rng.integers(len(RAMPS)))]
    if kind == PLAIN:
        return (O.FLAG_ZERO_LSB32 if rng.random() < 0.25 else 0), 256, ramp
    if kind == RAMPED:
        return O.FLAG_RAMP | (O.FLAG_ZERO_LSB32 if rng.random() < 0.25 else 0), 256, ramp
    if kind == SILENT:
        return O.FLAG_SILENCE, 256, ramp
    return (O.FLAG_RAMP if rng.random() < 0.5 else 0), int(rng.choice([100, 0, 1, 255, 64])), ramp


class PcmCase:
    def __init__(self, label, rows, src_bytes, dst_bytes, seed, counts):
        self.label, self.dst_bytes, self.counts = label, dst_bytes, counts
        self.descs = np.array(rows, dtype=O.MSG_DESC)
        self.src = np.random.default_rng(seed).integers(0, 256, size=max(src_bytes, 1), dtype=np.uint8)
        self._want = None

    def want(self):
        """The oracle's whole destination arena, one call (computed once)."""
        if self._want is None:
            dst = np.full(self.dst_bytes, FILL, dtype=np.uint8)
            assert O.msg_process_batch(self.descs, self.src, dst) == 0, self.label
            dst.setflags(write=False)
            self._want = dst
        return self._want

    def sampled(self):
        return range(0, self.descs.size, SAMPLE_EVERY)


@functools.lru_cache(maxsize=None)
def pcm_staged(cus):
    """List 0 of the line kernel: every message has 8-bit audio on one side at least, so every chunk is staged through `s_in`.
    One to three frames of 1-8 channels, plain / ramped / silent (and attenuated from 16 bits), both byte orders, every source
    offset mod 16; at seeded intervals of 24-48 chunks one message of 512 subsamples whose source is 1-4 bytes wide: stage_in issues
    1, 2 or 3 loads for it (3 = the 2304-byte buffer's most), none for a silent chunk -- the four `vmcnt` branches of the trip
    before it.  counts: chunks (sum of ceil(subsamples / 512)), loads (the set of load counts among the chunks)."""
    rng = np.random.default_rng(71000 + cus)
    need = staged_need(cus)
    rows, sp, dp, chunks, loads, residues = [], 0, 3, 0, set(), set()
    next_big = int(rng.integers(24, 48))
    while chunks <= need:
        big = chunks >= next_big
        if big:
            next_big = chunks + int(rng.integers(24, 48))
        if rng.random() < 0.5 and not big:
            sbits, dbits = 8, int(rng.choice([8, 16, 24, 32]))
        else:
            sbits, dbits = int(rng.choice([8, 16, 24, 32] if big else [16, 24, 32])), 8
        kinds = [PLAIN, RAMPED] + ([] if big else [SILENT, SILENT]) + ([ATTENUATED] if sbits == 16 else [])
        kind = kinds[int(rng.integers(len(kinds)))]
        ch = int(rng.choice([1, 2, 4, 8])) if big else int(rng.integers(1, 9))
        n = CHUNK_SUB // ch if big else int(rng.integers(1, 4))
        flags, att, ramp = _msg_fields(rng, kind)
        sp += int(rng.integers(0, 16))
        dp += int(rng.integers(0, 3))
        rows.append((sp, dp, n, ramp[0], ramp[1], att, ch, sbits, LE if rng.random() < 0.5 else BE, dbits, LE if rng.random() < 0.5 else BE, flags))
        loads.add(0 if kind == SILENT else stage_loads(sp, n * ch * sbits // 8))
        residues.add(sp % 16)
        chunks += (n * ch + CHUNK_SUB - 1) // CHUNK_SUB
        sp += n * ch * sbits // 8
        dp += n * ch * dbits // 8
    return PcmCase(f"staged list, {chunks} chunks", rows, sp, dp + 5, 71001 + cus, dict(chunks=chunks, loads=loads, residues=residues, need=need))


REGISTER_LISTS = {"16to24_heavy": (16, 24), "24to24_plain": (24, 24), "32to24_mixed": (32, 24)}


@functools.lru_cache(maxsize=None)
def pcm_register(cus, which):
    """One register list of the line kernel (one launch of pcm_line_kernel<S, D>), an ODD number of chunks so that the last trip's
    second chunk is missing for one wave.  One to five frames of 1-8 channels per message, one chunk per message:
      16to24_heavy   every message ramped or attenuated (a ramped / attenuated message is one chunk whatever its neighbours);
      24to24_plain   plain messages with 1-3 untouched bytes between them in both arenas, so that the planner cannot append one to
                     the other; at least four subsamples each (a run shorter than a group is not re-cut by the rule that cuts
                     merged runs near 4096 subsamples, but that rule is tests/test_gpu_pcm_textbook.py's to pin down);
      32to24_mixed   plain ones as above and ramped ones, shuffled.
    counts: group (plain chunks), heavy (ramped / attenuated chunks)."""
    sbits, dbits = REGISTER_LISTS[which]
    rng = np.random.default_rng(72000 + cus + sbits)
    need = register_need(cus)
    n_msgs = need + 1 + need % 2                                          # odd, and more than `need`
    rows, sp, dp, group, heavy = [], 1, 2, 0, 0
    for _ in range(n_msgs):
        if which == "16to24_heavy":
            kind = RAMPED if rng.random() < 0.6 else ATTENUATED
        elif which == "24to24_plain":
            kind = PLAIN
        else:
            kind = RAMPED if rng.random() < 0.4 else PLAIN
        ch, n = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        if kind == PLAIN and n * ch < 4:
            n = 4
        flags, att, ramp = _msg_fields(rng, kind)
        sp += int(rng.integers(1, 4))
        dp += int(rng.integers(1, 4))
        rows.append((sp, dp, n, ramp[0], ramp[1], att, ch, sbits, LE if rng.random() < 0.5 else BE, dbits, LE if rng.random() < 0.5 else BE, flags))
        group += kind == PLAIN
        heavy += kind != PLAIN
        sp += n * ch * sbits // 8
        dp += n * ch * dbits // 8
    return PcmCase(f"register list {which}, {n_msgs} chunks", rows, sp, dp + 3, 72001 + cus + sbits, dict(group=group, heavy=heavy, need=need))


# ---------------------------------------------------------------- Songcast frames (csrc/ohm_frame_kernel.hip)
OHM_WIDE_GROUPS_PER_CU = 4  # ohm_wide_kernel's cap today: 4 workgroups of 4 waves per CU, one record per wave


def ohm_narrow_need(cus):
    """Item 3a: a mono / stereo frame of one fragment is one prefixed chunk of the line kernel's register list for ITS depth (a list
    per source and wire depth, each list a launch of its own: 16 -> 16, 24 -> 24, 32 -> 24), two chunks per wave and trip; more than
    two trips for every wave of that launch, and a remainder that leaves some waves a third.  The condition is
    per list, so a case holds one depth."""
    return 2 * 2 * line_waves(cus) + 67


def ohm_wide_need(cus):
    """Item 3b: one record per wave; max(4 x 4 per CU today, 32 resident) waves, more than two trips each."""
    return 2 * max(OHM_WIDE_GROUPS_PER_CU * 4, MAX_WAVES_PER_CU) * cus + 67


class OhmCase:
    """Streams, frames of ONE fragment each and the fragments, the source arena, and the expected destination arena from the
    oracle: every fragment through ohp_msg_process_batch (one call, as a message to its own depth, big-endian), ohp_sender_pack,
    ohp_ohm_audio_frame."""

    def __init__(self, label, seed, formats, n_frames, kinds_of):
        rng = np.random.default_rng(seed)
        self.label, self.n = label, n_frames
        self.streams = np.zeros(len(formats), dtype=capi.OHM_STREAM)
        self.meta = []
        for i, (rate, bits, ch, endian) in enumerate(formats):
            codec = bytes(rng.integers(65, 91, int(rng.integers(0, 30)), dtype=np.uint8))
            s = self.streams[i]
            s["samples_total"], s["sample_rate"], s["bit_rate"] = int(rng.integers(0, 1 << 40)), rate, rate * bits * ch
            s["volume_offset"] = int(rng.integers(-300, 300))
            s["src_channels"], s["src_bits"], s["codec_bytes"], s["src_endian"] = ch, bits, len(codec), endian
            s["codec"][:len(codec)] = np.frombuffer(codec, dtype=np.uint8)
            self.meta.append(dict(rate=rate, bits=bits, ch=ch, endian=endian, codec=codec, kinds=kinds_of(bits, ch)))
        self.frames = np.zeros(n_frames, dtype=capi.OHM_FRAME_DESC)
        self.fragments = np.zeros(n_frames, dtype=capi.OHM_FRAGMENT)
        self.msgs = np.zeros(n_frames, dtype=O.MSG_DESC)                # the fragments as messages to their own depth, big-endian
        sp = tp = 0
        which = rng.integers(0, len(formats), n_frames)
        for k in range(n_frames):
            m = self.meta[int(which[k])]
            n = int(rng.integers(1, 4))
            kind = m["kinds"][int(rng.integers(len(m["kinds"])))]
            g, fr, d = self.fragments[k], self.frames[k], self.msgs[k]
            g["n_frames"], g["attenuation"] = n, 256
            if kind == RAMPED:
                g["flags"] = O.FLAG_RAMP
                g["ramp_start"], g["ramp_end"] = RAMPS[int(rng.integers(len(RAMPS)))]
            elif kind == SILENT:
                g["flags"] = O.FLAG_SILENCE
            elif kind == ATTENUATED:
                g["attenuation"] = int(rng.choice([100, 0, 255, 1]))
            nbytes = n * m["ch"] * m["bits"] // 8
            if kind != SILENT:
                sp += int(rng.integers(0, 5))
                g["src_offset"] = sp
                sp += nbytes
            d["src_offset"], d["dst_offset"], d["n_frames"] = int(g["src_offset"]), tp, n
            d["ramp_start"], d["ramp_end"], d["attenuation"], d["flags"] = g["ramp_start"], g["ramp_end"], g["attenuation"], g["flags"]
            d["channels"], d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"] = m["ch"], m["bits"], m["endian"], m["bits"], BE
            tp += nbytes
            fr["stream"], fr["frame"], fr["sample_start"] = int(which[k]), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 40))
            fr["network_timestamp"], fr["media_latency"] = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
            fr["first_fragment"], fr["n_fragments"] = k, 1
            fr["flags"] = capi.OHM_FLAG_LOSSLESS | (capi.OHM_FLAG_TIMESTAMPED if rng.random() < 0.3 else 0) | (capi.OHM_FLAG_HALT if rng.random() < 0.02 else 0)
        self.src = np.random.default_rng(seed + 1).integers(0, 256, size=max(sp, 1), dtype=np.uint8)
        self.tmp_bytes = tp
        self.gaps = rng.integers(0, 4, n_frames)
        self.records = int(((self.fragments["flags"] & O.FLAG_SILENCE) == 0).sum())     # the fragments with audio to read
        self._want = None

    def _headers(self):
        out = []
        for i, m in enumerate(self.meta):
            s = self.streams[i]
            wire_ch, wire_bits = OT.wire_format(m["ch"], m["bits"])
            n, sh = O.ohm_stream_header(int(s["samples_total"]), m["rate"], int(s["bit_rate"]), int(s["volume_offset"]), wire_bits, wire_ch, m["codec"])
            assert n == 22 + len(m["codec"])
            out.append(sh)
        return out

    def want(self):
        """(frames with their dst_offset filled in, the whole destination arena, its size); computed once."""
        if self._want is None:
            import ctypes as C
            pcm = np.zeros(max(self.tmp_bytes, 1), dtype=np.uint8)
            assert O.msg_process_batch(self.msgs, self.src, pcm) == 0, self.label
            headers, grams, at = self._headers(), [], 3
            packed, nb = np.zeros(8192, dtype=np.uint8), C.c_uint32(0)
            for k in range(self.n):
                d, fr = self.msgs[k], self.frames[k]
                ch, nbytes, n = int(d["channels"]), int(d["src_bits"]) // 8, int(d["n_frames"])
                piece = np.ascontiguousarray(pcm[int(d["dst_offset"]):int(d["dst_offset"]) + n * ch * nbytes])
                assert O.lib().ohp_sender_pack(O._ptr(piece), piece.size, ch, nbytes, O._ptr(packed), C.byref(nb)) == 0
                size, gram = O.ohm_audio_frame(int(fr["flags"]), n, int(fr["frame"]), int(fr["network_timestamp"]), int(fr["media_latency"]),
                                               int(fr["sample_start"]), headers[int(fr["stream"])], packed[:nb.value].tobytes())
                assert size == gram.size > 0, (self.label, k, size)
                fr["dst_offset"] = at
                grams.append((at, gram))
                at += gram.size + int(self.gaps[k])
            dst = np.full(at + 3, FILL, dtype=np.uint8)
            for off, gram in grams:
                dst[off:off + gram.size] = gram
            dst.setflags(write=False)
            self._want = (self.frames, dst, at + 3, grams)
        return self._want


def _narrow_kinds(bits, ch):
    return [PLAIN, PLAIN, RAMPED, SILENT] + ([ATTENUATED] if bits == 16 else [])


def _wide_kinds(bits, ch):
    return [PLAIN, PLAIN, PLAIN, RAMPED, SILENT] + ([ATTENUATED] if bits == 16 else [])


OHM_NARROW_BITS = (16, 24, 32)


@functools.lru_cache(maxsize=None)
def ohm_narrow(cus, bits):
    """Mono and stereo streams of ONE depth (16, 24 or 32 bits: one register list of the line kernel, hence one launch, a header
    prefix on every chunk), both source byte orders, codec names of 0-29 bytes (prefixes of 58-87 bytes), frames of one fragment of
    one to three audio frames; silent fragments ride in the same list."""
    formats = [(rate, bits, ch, endian) for ch in (1, 2) for rate, endian in ((44100, BE), (48000, LE), (96000, BE))]
    n = ohm_narrow_need(cus) + 1
    return OhmCase(f"{n} mono / stereo frames of {bits} bits", 73000 + cus + bits, formats, n, _narrow_kinds)


@functools.lru_cache(maxsize=None)
def ohm_wide(cus):
    """Six- and eight-channel streams of every depth: one record of ohm_wide_kernel per fragment that has audio (`records`; a
    silent fragment reads none and is written with the headers) -- a third more frames than the condition needs, one in five or
    six of them silent; ramped and (at 16 bits) attenuated fragments among the plain ones."""
    formats = [(48000, bits, ch, LE if (bits // 8 + ch) % 2 else BE) for bits in (8, 16, 24, 32) for ch in (6, 8)]
    n = ohm_wide_need(cus) * 4 // 3 + 1
    return OhmCase(f"{n} six- and eight-channel frames", 73500 + cus, formats, n, _wide_kinds)


# ---------------------------------------------------------------- DSD -> PCM (csrc/dsd_pcm_kernel.hip)
DSD_PCM_TILE = 512          # kDsdPcmTile: frames per tile
DSD_PCM_KEY = (32, 16)


def dsd_pcm_need(cus, route):
    """Both kernels take one tile per 1024-thread workgroup (kDsdPcmThreads: 16 waves), so a CU keeps floor(32 / 16) = 2 resident.
    fast: max(today's occupancy <= 2 per CU, 2) x CUs workgroups, more than three trips; plain: max(today's cap of 8 per CU at the
    launch site, 2) x CUs -- the 8 is the cap, not residency -- more than two trips."""
    return 3 * 2 * cus + 37 if route == "fast" else 2 * 8 * cus + 37


@functools.lru_cache(maxsize=None)
def dsd_pcm(cus):
    """One batch for both routes (its tiles outnumber the larger of the two conditions): messages of 1-5 frames and, at seeded
    intervals of 20-60 messages, one of 512 frames -- a full tile before a short one in the same `stage`; out_frame0 of all three
    classes (0 puts the 0x69 lead-in into a stage that just held real bytes), every (W, P), both byte orders, one in six ramped.
    Returns (case, tiles)."""
    rng = np.random.default_rng(74000 + cus)
    need = max(dsd_pcm_need(cus, "fast"), dsd_pcm_need(cus, "plain"))
    b = DC.Batch(DSD_PCM_KEY, 74001 + cus, src_lead=1, dst_lead=3)
    tiles, next_full = 0, int(rng.integers(20, 60))
    while tiles <= need:
        full = tiles >= next_full
        if full:
            next_full = tiles + int(rng.integers(20, 60))
        n = DSD_PCM_TILE if full else int(rng.integers(1, 6))
        kind = "noise" if rng.random() < 0.85 else DC.INPUTS[int(rng.integers(1, len(DC.INPUTS)))]
        b.add(int(rng.choice(DC.OUT0)), n, DC.FORMATS[int(rng.integers(3))], kind, RAMPS[int(rng.integers(len(RAMPS)))] if rng.random() < 1 / 6 else None,
              capi.ENDIAN_LITTLE if rng.random() < 0.5 else capi.ENDIAN_BIG, src_gap=int(rng.integers(0, 3)), dst_gap=int(rng.integers(0, 3)))
        tiles += (n + DSD_PCM_TILE - 1) // DSD_PCM_TILE
    return b.finish(f"{tiles} tiles", dst_tail=5), tiles


# ---------------------------------------------------------------- the pulled resampler (csrc/src_pull_kernel.hip)
PULL_S = 8


def pull_need(cus):
    """One tile per 256-thread workgroup (4 waves): max(today's occupancy x CUs <= 8 per CU, floor(32 / 4) = 8) x CUs workgroups,
    more than three trips."""
    return 3 * 8 * cus + 37


class PullCase:
    def __init__(self, label, T, descs, src, dst_bytes):
        self.label, self.T, self.descs, self.src, self.dst_bytes = label, T, descs, src, dst_bytes
        self._want = None

    def table(self):
        return pull_table(self.T)

    def want(self, ramp_table):
        """tests/src_pull_model.py message by message (computed once)."""
        if self._want is None:
            dst = np.full(self.dst_bytes, FILL, dtype=np.uint8)
            for d in self.descs:
                out = PM.message_bytes(self.table(), PULL_S, d, self.src, ramp_table)
                dst[int(d["dst_offset"]):int(d["dst_offset"]) + out.size] = out
            dst.setflags(write=False)
            self._want = dst
        return self._want


@functools.lru_cache(maxsize=None)
def pull_table(T):
    return capi.src_pull_design(44100, 48000, T, PULL_S, 8.0 if T == 32 else 9.0, 20000.0, 0.001)


@functools.lru_cache(maxsize=None)
def pull(cus, stereo_only, T):
    """Messages of 1-5 outputs, each with its own packed window and pull (a tile never spans messages, so the messages are a lower
    bound of the tiles); at seeded intervals of 30-90 one of 256 outputs, whose window of about 270 frames is near (eight channels:
    beyond) what the LDS holds; one in ten a stream start.  Mixed: 1-8 channels, 8 / 16 / 24 / 32-bit sources in both orders, 16 /
    24 / 32-bit destinations in both orders, one in six ramped, ZERO_LSB32 on a quarter -- src_pull_kernel<0>, the layout changing
    from tile to tile.  Stereo only: the same with two channels everywhere -- src_pull_kernel<2>."""
    rng = np.random.default_rng(75000 + cus + T + (1 if stereo_only else 0))
    need = pull_need(cus)
    descs = np.zeros(need + 1, dtype=capi.SRC_PULL_MSG_DESC)
    src, sp, dp, next_long = [], 0, 1, int(rng.integers(30, 90))
    for k in range(need + 1):
        long_one = k >= next_long
        if long_one:
            next_long = k + int(rng.integers(30, 90))
        n = 256 if long_one else int(rng.integers(1, 6))
        ch = 2 if stereo_only else int(rng.integers(1, 9))
        sb, db = int(rng.choice([8, 16, 24, 32])), int(rng.choice([16, 24, 32]))
        step = PM.step_of(44100, 48000, PM.multiplier_of(int(rng.integers(-1000, 1001))))
        if rng.random() < 0.1:
            pos, frac = 0, 0
        else:
            pos, frac = int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 32))
        first, frames = PM.window(pos, frac, step, n, T)
        data = rng.integers(0, 256, size=frames * ch * sb // 8, dtype=np.uint8)
        src += [data, np.zeros(-data.size % 16, dtype=np.uint8)]
        d = descs[k]
        d["src_offset"], d["src_frame0"], d["src_frames"] = sp, first, frames
        d["pos_frame"], d["pos_frac"], d["step"], d["n_frames"] = pos, frac, step, n
        dp += int(rng.integers(0, 3))
        d["dst_offset"], d["attenuation"] = dp, capi.UNITY_ATTENUATION
        d["ramp_start"], d["ramp_end"] = RAMPS[int(rng.integers(len(RAMPS)))]
        d["channels"], d["src_bits"], d["src_endian"] = ch, sb, LE if rng.random() < 0.5 else BE
        d["dst_bits"], d["dst_endian"] = db, LE if rng.random() < 0.5 else BE
        d["flags"] = (capi.FLAG_RAMP if rng.random() < 1 / 6 else 0) | (capi.FLAG_ZERO_LSB32 if rng.random() < 0.25 else 0)
        sp += data.size + (-data.size % 16)
        dp += n * ch * db // 8
    what = "stereo" if stereo_only else "mixed"
    return PullCase(f"pulled {what} T={T}, {need + 1} messages", T, descs, np.concatenate(src), dp + 3)


# ---------------------------------------------------------------- the block resamplers (csrc/src_lean_kernel.hip, src_block_kernel.hip, src_mfma_wg_kernel.hip)
F44, F96 = (44100, 48000, 32), (96000, 48000, 64)
F44_LOUD = (44100, 48000, 32, 65)      # the same design with every coefficient times 65 / 64: see src_filter
WG, LEAN, BLOCK = "src_mfma_wg_kernel", "src_lean_kernel", "src_block_kernel"
# src_block_kernel (round 1's, the fallback for a filter beyond the lean kernel's rounding bound: sum|c| >= 2^29 in a phase) serves 48 ->
# 44.1 kHz, whose design has 2.018 x 2^28 in its heaviest phase.  That ratio's block is whole phase periods AND whole 64-byte output
# lines (src_block_outputs_for): 147 x 32 = 4704 outputs, so 2 x 32 x CUs one-block units would be half a gigabyte in each arena.
# The same kernel, claim loop and counters are reached with 160-output blocks by the 44.1 -> 48 kHz design (1.992 x 2^28) at a gain
# of 65 / 64 (2.023 x 2^28): "stereo_s24_block" below, under the default variant.
# (filter, (channels, source bits, source order, destination bits, destination order), [(kernel variant, the kernel it must run on)])
SRC_CASES = {
    "stereo_s24": (F44, (2, 24, LE, 24, BE), [(0, WG), (4, LEAN), (2, LEAN)]),
    "halfband_stereo": (F96, (2, 24, LE, 24, BE), [(0, WG), (4, LEAN)]),
    "six_s24": (F44, (6, 24, LE, 24, BE), [(0, WG), (4, LEAN)]),
    "stereo_to_s16": (F44, (2, 24, LE, 16, BE), [(0, LEAN)]),
    "stereo_s24_block": (F44_LOUD, (2, 24, LE, 24, BE), [(0, BLOCK)]),
}
SRC_BLOCK_OUT = 160


def src_need(cus):
    """Units of the block resamplers: one per wave (lean: CUs x <= 12 waves today) or per workgroup (matrix kernel:
    3 x CUs today); against the 32 waves a CU keeps resident, more than two trips: 2 x 32 x CUs."""
    return 2 * MAX_WAVES_PER_CU * cus


class SrcCase:
    def __init__(self, label, flt, lay, descs, src, dst_bytes, n_streams):
        self.label, self.flt, self.lay, self.descs, self.src, self.dst_bytes, self.n_streams = label, flt, lay, descs, src, dst_bytes, n_streams
        self._want = None

    def ref(self):
        return src_ref(self.flt)

    def want(self):
        """The oracle's whole destination arena (O.Src.process_batch; computed once)."""
        if self._want is None:
            dst = np.full(self.dst_bytes, FILL, dtype=np.uint8)
            assert self.ref().process_batch(self.descs, self.src, dst) == 0, self.label
            dst.setflags(write=False)
            self._want = dst
        return self._want


@functools.lru_cache(maxsize=None)
def src_filter(flt):
    """(L, M, the Q28 coefficients) of capi.src_design(rate in, rate out, taps, 9.0, 20000.0); with a fourth entry g the
    coefficients are floor(c x g / 64), which for g = 65 takes the heaviest phase's sum|c| over the lean kernel's 2^29."""
    L, M, coef = capi.src_design(flt[0], flt[1], flt[2], 9.0, 20000.0)
    if len(flt) > 3:
        coef = ((np.asarray(coef, dtype=np.int64) * flt[3]) >> 6).astype(np.int32)
        heaviest = int(np.abs(coef.astype(np.int64)).reshape(L, flt[2]).sum(axis=1).max())
        assert 1 << 29 <= heaviest < 1 << 30, heaviest
    return L, M, coef


@functools.lru_cache(maxsize=None)
def src_ref(flt):
    ref = O.Src(flt[0], flt[1], flt[2], 9.0, 20000.0)
    if len(flt) > 3:
        ref.set_coef_q28(src_filter(flt)[2])
    return ref


@functools.lru_cache(maxsize=None)
def src_streams(cus, name):
    """Many short streams of one layout, a unit each (a unit's rows are blocks of ONE stream, so a stream of fewer blocks than a
    unit has rows is one partly filled unit): one to three blocks of 160 outputs (four in five have one) and a ragged tail of 0-47
    outputs for the generic kernel, in messages of up to 240 frames; one stream in fifty is asked for from an output past its
    first, one message in a hundred is ramped.  Five in a hundred more streams than the condition needs."""
    flt, lay, _ = SRC_CASES[name]
    ch, sb, se, db, de = lay
    ref = src_ref(flt)
    rng = np.random.default_rng(76000 + cus + sum(name.encode()))
    n_streams = src_need(cus) + src_need(cus) // 20 + 1
    fb_src, fb_dst = ch * sb // 8, ch * db // 8
    rows, sp, dp = [], 0, 0
    for _ in range(n_streams):
        blocks = int(rng.choice([1, 1, 1, 1, 2, 2, 3, 1, 1, 1]))
        out0 = int(rng.integers(1, 300)) if rng.random() < 0.02 else 0
        end = out0 + blocks * SRC_BLOCK_OUT + int(rng.integers(0, 48)) + (2 * SRC_BLOCK_OUT if out0 else 0)
        in_frames = (end * ref.M + ref.L - 1) // ref.L + 1
        while ref.out_frames(in_frames) < end:
            in_frames += 1
        dp += int(rng.integers(0, 4))
        m = out0
        while m < end:
            n = min(240, end - m)
            ramp = RAMPS[int(rng.integers(len(RAMPS)))]
            rows.append((sp, 0, in_frames, m, dp + (m - out0) * fb_dst, n, ramp[0], ramp[1], 256, ch, sb, se, db, de,
                         O.FLAG_RAMP if rng.random() < 0.01 else 0, 0))
            m += n
        sp += in_frames * fb_src
        dp += (end - out0) * fb_dst
    src = np.random.default_rng(76001 + cus).integers(0, 256, size=sp, dtype=np.uint8)
    return SrcCase(f"{name}: {n_streams} streams", flt, lay, np.array(rows, dtype=O.SRC_MSG_DESC), src, dp + 3, n_streams)


# ---------------------------------------------------------------- the FLAC scan's second attempt (csrc/flac_frame_kernel.hip, flac_run)
def flac_first_list(src_bytes):
    """The scan's first list: flac_run asks for S / 512 + 256 entries, and the block cache hands out half as much again plus 32.
    (If that sizing changes, this changes with it.)"""
    return 1.5 * (src_bytes / 512 + 256) + 32


@functools.lru_cache(maxsize=None)
def flac_cases():
    """256 descriptors over the six-frame tiny stream, planes and packed in turn, the eight-frame mono stream every 16th."""
    import flac_cases as FC
    tiny, forms = FC.fixture("tiny_s16_stereo_44k1_b16"), FC.fixture("forms_s16_mono_11k_b16")
    return tuple(FC.whole(forms, label=f"forms#{k}") if k % 16 == 15 else FC.whole(tiny, packed=bool(k % 2), label=f"tiny#{k}") for k in range(256))
