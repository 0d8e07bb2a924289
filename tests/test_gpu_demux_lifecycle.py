"""The shell every batch family of the C ABI shares (tests/test_gpu_batch_lifecycle.py), for the families whose signatures do not fit
that file's Case: DSD -> PCM (a filter in front of the descriptors), RAOP and the Songcast receiver (two tables), Ogg and MPEG-4 (a
packet table's size; MPEG-4 without a destination arena), PCM files and DSD files.  The same five things: what a failed create leaves behind,
what a run refuses (another family's batch, no batch, null arenas) and accepts (an empty batch), and that the host-buffer call equals
create + run on device arenas, keeps its hands off every byte no output covers, and moves exactly what the MODEL says was delivered.

The batches are the smallest valid ones of each family, two outputs each:

    dsd_pcm    D = 8, T = 8: a message of 16 frames from the stream's start and one of 5 frames from frame 7
    raop       a plaintext stream of one packet of 20 bytes, and tests/alac_cases.handmade's hand_stereo8 (one packet, eight samples)
               encrypted with the tests' own AES, decoded into planes
    ohm_rx     two streams of one audio datagram each (2 and 3 stereo 16-bit frames); the room is the datagram's length less the
               fixed header, four bytes more than the audio
    ogg        two streams of one page of one packet (10 and 11 bytes); the room is the stream's length, as the ABI asks
    mp4        two files of three and four packets; the "outputs" are their rows of the two tables, the hole is four rows
    iff        two 16-bit stereo WAV files of 4 and 5 frames
    dsd_file   a DSF file of 8 chunks and a DFF file of 4, into (W, P) = (2, 0): 32 and 16 bytes, so that every dst_offset is the
               multiple of 16 the family asks for
    mp4f       two gathered fragmented files of three and four samples in one run each; cenc: the same under two keys (8-byte IVs); cbcs:
               the same with two subsample entries a sample under the 1:1 pattern.  The outputs are the gathered (clear) bytes; each has
               a second case that gathers nothing (mp4f: no OHGPU_MP4F_GATHER; the protected families: no room), which runs without
               a destination arena
    vorbis     tests/vorbis_cases.py's mono_64_128, packets [0, 4) and [4, 9), packed 16-bit: the one family whose output is held to
               the model within 1 LSB (tests/test_gpu_vorbis_textbook.py) and to the device-arena run exactly
    ts, adts, raop_rx   (a failed create, null arenas and the empty batch alone: tests/test_gpu_ts_lifecycle.py and
               tests/test_gpu_raop_rx_lifecycle.py pin the rest) two small streams each

Every table passes the library's own check before it reaches a launch; the refusals are refused before anything is queued."""
import ctypes as C

import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T
import cbcs_cases as BC
import cbcs_textbook as BX
import cenc_cases as CC
import cenc_textbook as CX
import dsd_file_cases as FC
import dsd_file_textbook as FX
import dsd_pcm_cases as DC
import iff_cases as IC
import iff_textbook as IX
import mp4_cases as MC
import mp4_textbook as MX
import mp4f_cases as MF
import mp4f_textbook as MFX
import ogg_cases as GC
import ogg_textbook as OX
import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import raop_rx_cases as XC
import raop_textbook as R
import ts_cases as TC
import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

HOLE, HOLE_ROWS = 64, 4
DEV_FILL, HOST_FILL = 0xA5, 0x5A
ZERO_INFO = {"n_msgs": 0, "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}
FRAGMENTED = ("mp4f", "cenc", "cbcs")                                # their outputs are gathered bytes, and three tables beside them
FAMILIES = ("dsd_pcm", "raop", "ohm_rx", "ogg", "mp4", "iff", "dsd_file") + FRAGMENTED + ("vorbis",)
SHELL_ONLY = ("ts", "adts", "raop_rx")                               # a failed create, null arenas, the empty batch: what their own files lack
NO_ARENA = ("mp4", "adts", "raop_rx")                                # no destination arena: run(ctx, batch, src, stream)
# the text of run_guard's "<who>: not a <noun> batch" (csrc/ohgpu_api.hip: kKinds' nouns); MPEG-4 and PCM files word their own
NOT_MINE = {"dsd_pcm": "not a DSD to PCM batch", "raop": "not a RAOP batch", "ohm_rx": "not a Songcast receiver batch", "ogg": "not a Ogg batch",
            "mp4": "not an MPEG-4 batch", "iff": "not a PCM file batch", "dsd_file": "not a DSD file batch", "mp4f": "not a fragmented MPEG-4 batch",
            "cenc": "not a protected MPEG-4 batch", "cbcs": "not a cbcs-protected MPEG-4 batch", "vorbis": "not a Vorbis batch"}
# what last_error says of the last descriptor when its output lies past its arena (MPEG-4: its rows past the tables, its file past the arena)
BOUNDS_TEXT = {"dsd_pcm": "dsd pcm desc 1: writes [", "raop": "alac desc 1: writes [", "ohm_rx": "ohm rx stream 1: writes [", "ogg": "ogg desc 1: writes [",
               "iff": "iff desc 1: writes [", "dsd_file": "dsd file desc 1: writes [",
               # (the protected families' descriptors pass through ohgpu_mp4f_batch_check for the fields they share: csrc/api_cenc.hip, csrc/api_cbcs.hip)
               "mp4f": "mp4f desc 1: gathers into [", "cenc": "mp4f desc 1: gathers into [", "cbcs": "mp4f desc 1: gathers into [", "vorbis": "vorbis desc 1: writes [",
               "ts": "ts desc 1: writes [", "adts": "adts desc 1: reads [", "raop_rx": "raop rx stream 1: reads ["}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _offsets(sizes, hole):
    """Outputs back to back, `hole` between the first and the second."""
    at, out = 0, []
    for k, s in enumerate(sizes):
        out.append(at)
        at += s + (hole if k == 0 and len(sizes) > 1 else 0)
    return out, at


def _u8(raw):
    return np.frombuffer(bytes(raw), dtype=np.uint8).copy()


class Case:
    """One batch: `head` = the create call's arguments between the context and the arena sizes (`keep` holds their arrays), the source
    arena, the destination arena's size (None: the family has none), `pieces` = (offset, bytes) of everything the MODEL says a run
    delivers with `model` = those bytes, `moved` = the bytes the host-buffer call brings home, `tail` = that call's result arguments."""

    def __init__(self, family, head, keep, src, dst_bytes, pieces=(), moved=0, tail=(), out=(), want=()):
        self.family, self.head, self.keep, self.src, self.dst_bytes, self.pieces, self.moved, self.tail = family, head, keep, src, dst_bytes, list(pieces), moved, tail
        self.out, self.want = out, want         # the fragmented families: the arrays `tail` points into (results, runs, packets, samples), the model's three tables

    def sizes(self):
        return (self.src.size,) if self.dst_bytes is None else (self.src.size, self.dst_bytes)

    def arena(self, fill):
        """The destination arena the model leaves when it starts as `fill`."""
        out = np.full(self.dst_bytes, fill, dtype=np.uint8)
        for off, raw in self.pieces:
            out[off:off + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        return out


class Fixtures:
    def __init__(self):
        self.ctx = capi.Context(0)
        self.dsd_key = (8, 8)
        self.dsd_filter = self.ctx.dsd_pcm_create(*self.dsd_key, DC.coef(self.dsd_key))

    def close(self):
        self.ctx.dsd_pcm_destroy(self.dsd_filter)
        self.ctx.close()

    # ---- the families' smallest batches.  hole: between the first output and the second; bad: the last descriptor's output starts
    # where its arena ends ("rows" / "file" for MPEG-4); empty: no descriptors
    def case(self, family, hole=0, bad=None, empty=False, **more):
        return getattr(self, "_" + family)(0 if empty else 2, hole, bad, **more)

    def _dsd_pcm(self, n, hole, bad):
        b = DC.Batch(self.dsd_key, 9600)
        for out0, frames in ((0, 16), (7, 5))[:n]:
            b.add(out0, frames, dst_gap=hole if out0 else 0)
        c = b.finish("lifecycle")
        pieces = [(int(d["dst_offset"]), c.want()[int(d["dst_offset"]):int(d["dst_offset"]) + 6 * int(d["n_frames"])].tobytes()) for d in c.descs] if n else []
        if bad:
            c.descs["dst_offset"][-1] = c.dst_bytes
        # (this family's host-buffer call is the generic one: one copy of the covered span, the hole included)
        moved = max(o + len(r) for o, r in pieces) - min(o for o, _ in pieces) if n else 0
        return Case("dsd_pcm", (self.dsd_filter, _ptr(c.descs), n), [c.descs], c.src if n else np.zeros(0, np.uint8), c.dst_bytes, pieces, moved)

    def _raop(self, n, hole, bad):
        rng = AC.Lcg(71)
        keys = [(bytes(rng.next() & 0xff for _ in range(16)), bytes(rng.next() & 0xff for _ in range(16))) for _ in range(2)]
        cookie, (packet,) = AC.handmade()["hand_stereo8"]
        cfg = T.parse_config(cookie)
        clear = bytes(rng.next() & 0xff for _ in range(20))
        payloads = [R.encrypt_packet(*keys[0], clear), R.encrypt_packet(*keys[1], packet)][:n]
        each = [20, 2 * cfg["frame_length"] * 4]                    # the packet's bytes; two planes of one packet's frame length
        offs, dst_bytes = _offsets(each[:n], hole)
        descs, packets, src = np.zeros(n, dtype=capi.RAOP_STREAM_DESC), np.zeros(n, dtype=capi.ALAC_PACKET), bytearray()
        for i in range(n):
            src += bytes(-len(src) % 4)
            packets[i]["src_offset"], packets[i]["bytes"] = len(src), len(payloads[i])
            src += payloads[i]
            descs[i]["first_packet"], descs[i]["n_packets"], descs[i]["dst_offset"] = i, 1, offs[i]
            descs[i]["aes_key"], descs[i]["aes_iv"] = list(keys[i][0]), list(keys[i][1])
        pieces = []
        if n:
            descs[0]["flags"] = capi.RAOP_OUT_PLAINTEXT
            for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
                descs[1][k] = cfg[k]
            descs[1]["dst_plane_stride"] = cfg["frame_length"] * 4
            planes = bytearray(bytes([DEV_FILL]) * (offs[1] + each[1]))
            assert [tuple(w) for w in T.render(cfg, [packet], T.PLANAR, planes, offs[1], cfg["frame_length"] * 4, decode_packet=AC.decode_cached)] == [(T.OK, 8)]
            pieces = [(offs[0], clear)] + [(offs[1] + c * cfg["frame_length"] * 4, bytes(planes[offs[1] + c * cfg["frame_length"] * 4:][:8 * 4])) for c in range(2)]
        if bad:
            descs["dst_offset"][-1] = dst_bytes
        self.raop_results = (np.zeros(n, dtype=capi.ALAC_STREAM_RESULT), np.zeros(n, dtype=capi.ALAC_PACKET_RESULT))
        return Case("raop", (_ptr(descs), n, _ptr(packets), n), [descs, packets], _u8(src), dst_bytes, pieces, sum(len(r) for _, r in pieces),
                    tuple(_ptr(a) for a in self.raop_results))

    def _ohm_rx(self, n, hole, bad):
        rng = RC.Lcg(72)
        grams = [RC.audio_gram(5 + i, rng.bytes(4 * (2 + i))) for i in range(n)]
        offs, dst_bytes = _offsets([len(g) - 58 for g in grams], hole)
        streams, table, src, pieces = np.zeros(n, dtype=capi.OHM_RX_STREAM), np.zeros(n, dtype=capi.OHM_RX_DATAGRAM), bytearray(), []
        for i, g in enumerate(grams):
            src += bytes(-len(src) % 4)
            table[i]["src_offset"], table[i]["bytes"] = len(src), len(g)
            src += g
            streams[i]["first_datagram"], streams[i]["n_datagrams"], streams[i]["dst_offset"], streams[i]["dst_capacity"] = i, 1, offs[i], len(g) - 58
            RC.state_row(streams[i], "", RX.new_state())
            _, res, out = RX.receive(RX.new_state(), [g], offs[i])
            assert res["out_bytes"] == len(out) == 4 * (2 + i) < len(g) - 58
            pieces.append((offs[i], bytes(out)))
        if bad:
            streams["dst_offset"][-1] = dst_bytes
        return Case("ohm_rx", (_ptr(streams), n, _ptr(table), n), [streams, table], _u8(src), dst_bytes, pieces, sum(len(r) for _, r in pieces), (None, None))

    def _ogg(self, n, hole, bad):
        rng = GC.Lcg(73)
        data = [GC.page(7, 0, [10 + i], rng.bytes(10 + i), OX.BOS | OX.EOS, 1) for i in range(n)]
        offs, dst_bytes = _offsets([len(d) for d in data], hole)
        descs, src, pieces = np.zeros(n, dtype=capi.OGG_STREAM_DESC), bytearray(), []
        for i, d in enumerate(data):
            descs[i]["src_offset"], descs[i]["src_bytes"], descs[i]["dst_offset"], descs[i]["dst_capacity"] = len(src), len(d), offs[i], len(d)
            descs[i]["serial"], descs[i]["packet_first"], descs[i]["packet_capacity"] = 7, i, 1
            src += d
            m = OX.demux(d, 7, 0, 0, 0)
            assert m["status"] == OX.OK and len(m["run"]) == 10 + i
            pieces.append((offs[i], bytes(m["run"])))
        if bad:
            descs["dst_offset"][-1] = dst_bytes
        return Case("ogg", (_ptr(descs), n, n), [descs], _u8(src), dst_bytes, pieces, sum(len(r) for _, r in pieces), (None, None))

    def _mp4(self, n, hole, bad):
        files = [MC.mux(MC.pattern_packets(3 + i, seed=1 + i), MC.PATTERN_COOKIE) for i in range(n)]
        firsts, rows = _offsets([m.n for m in files], HOLE_ROWS if hole else 0)
        descs, src = np.zeros(n, dtype=capi.MP4_STREAM_DESC), bytearray()
        self.mp4_want = (np.frombuffer(bytes([DEV_FILL]) * (16 * rows), dtype=capi.ALAC_PACKET).copy(), np.frombuffer(bytes([DEV_FILL]) * (16 * rows), dtype=capi.MP4_SAMPLE).copy())
        for i, m in enumerate(files):
            descs[i]["src_offset"], descs[i]["src_bytes"], descs[i]["packet_first"], descs[i]["packet_capacity"] = len(src), len(m.data), firsts[i], m.n
            model = MX.demux(m.data, m.n)
            MC.check_against_record(model, m)
            for s, (row, sample) in enumerate(zip(model["rows"], model["samples_rows"])):       # (as tests/mp4_cases.Job lays them)
                self.mp4_want[0][firsts[i] + s] = (len(src) + row[0], row[1], 0)
                self.mp4_want[1][firsts[i] + s] = sample
            src += m.data
        if bad == "rows":
            descs["packet_first"][-1] = rows
        elif bad:
            descs["src_offset"][-1] = len(src)
        self.mp4_results = (np.zeros(n, dtype=capi.MP4_STREAM_RESULT), np.zeros(rows, dtype=capi.ALAC_PACKET), np.zeros(rows, dtype=capi.MP4_SAMPLE))
        return Case("mp4", (_ptr(descs), n, rows), [descs], _u8(src), None, tail=tuple(_ptr(a) for a in self.mp4_results))

    def _iff(self, n, hole, bad):
        files = [IC.wav(IC.samples(4 + i, 2, 2, 40 + i), 2) for i in range(n)]
        offs, dst_bytes = _offsets([w.frames * 4 for w in files], hole)
        descs, src, pieces = np.zeros(n, dtype=capi.IFF_STREAM_DESC), bytearray(), []
        for i, w in enumerate(files):
            d = descs[i]
            d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_bytes_capacity"], d["dst_frame_capacity"], d["max_bit_depth"] = len(src), len(w.data), offs[i], w.frames * 4, w.frames, 24
            src += w.data
            m = IX.read(w.data, dst_frame_capacity=w.frames, dst_bytes_capacity=w.frames * 4)
            IC.check_against_record(m, w)
            pieces.append((offs[i], bytes(m["pcm"])))
        if bad:
            descs["dst_offset"][-1] = dst_bytes
        return Case("iff", (_ptr(descs), n), [descs], _u8(src), dst_bytes, pieces, sum(len(r) for _, r in pieces), (None,))

    def _dsd_file(self, n, hole, bad):
        files = [FC.make(kind, chunks, 50 + i) for i, (kind, chunks) in enumerate(((FX.DSF, 8), (FX.DFF, 4))[:n])]
        offs, dst_bytes = _offsets([w.chunks_total // 2 * 8 for w in files], hole)         # (W, P) = (2, 0): two chunks to a block of 8 bytes
        descs, src, pieces = np.zeros(n, dtype=capi.DSD_FILE_STREAM_DESC), bytearray(), []
        for i, w in enumerate(files):
            d, room = descs[i], w.chunks_total // 2 * 8
            d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_bytes_capacity"], d["sample_block_words"], d["pad_bytes_per_chunk"] = len(src), len(w.data), offs[i], room, 2, 0
            src += w.data
            m = FX.read(w.data, 2, 0, dst_bytes_capacity=room)
            assert m["status"] == FX.OK and m["chunks_written"] == w.chunks_total and m["bytes_written"] == len(m["blocks"]) == room
            pieces.append((offs[i], bytes(m["blocks"])))
        if bad:
            descs["dst_offset"][-1] = dst_bytes
        return Case("dsd_file", (_ptr(descs), n), [descs], _u8(src), dst_bytes, pieces, sum(len(r) for _, r in pieces), (None,))

    def _frag_file(self, family, i):
        if family == "mp4f":
            return MF.simple([3 + i], seed=1 + i)
        if family == "cenc":
            return CC.simple([3 + i], seed=1 + i, iv_size=8, key=CC.key_of(i), kid=CC.kid_of(i))
        parts = [[(3 + k, 16 * (k + 1) + 5), (0, 16)] for k in range(3 + i)]
        return BC.build([sum(c + q for c, q in e) for e in parts], iv_size=16, pattern=(1, 1), layout=BC.split_layout(parts), seed=1 + i, key=BC.key_of(i), kid=BC.kid_of(i))

    def _frag(self, family, n, hole, bad, gather=True):
        """gather=False: the same files with nothing to gather (mp4f: the flag is off; the protected families always carry it: no room)"""
        files = [self._frag_file(family, i) for i in range(n)]
        clear = [sum(m.sizes) for m in files]
        offs, dst_bytes = _offsets(clear, hole)
        firsts, rows = _offsets([m.n for m in files], HOLE_ROWS if hole else 0)
        run_firsts, runs = _offsets([len(m.runs) for m in files], HOLE_ROWS if hole else 0)
        sub_firsts, subs = _offsets([m.subsamples for m in files], HOLE_ROWS if hole else 0) if family == "cbcs" else (None, 0)
        descs = np.zeros(n, dtype={"mp4f": capi.MP4F_STREAM_DESC, "cenc": capi.CENC_STREAM_DESC, "cbcs": capi.CBCS_STREAM_DESC}[family])
        src, pieces = bytearray(), []
        want = tuple(np.frombuffer(bytes([DEV_FILL]) * (t.itemsize * k), dtype=t).copy() for t, k in ((capi.MP4F_RUN, runs), (capi.ALAC_PACKET, rows), (capi.MP4_SAMPLE, rows)))
        for i, m in enumerate(files):
            d, room = descs[i], clear[i] if gather else 0
            d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = len(src), len(m.data), 3, 1 if gather or family != "mp4f" else 0
            d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = firsts[i], m.n, run_firsts[i], len(m.runs)
            d["dst_offset"], d["dst_capacity"] = (offs[i], room) if gather else (0, 0)
            if family == "mp4f":
                model = MFX.demux(m.data, 3, m.n, len(m.runs), gather, 0, room)
                MF.check_against_record(model, m)
                places = [(len(src) + r[0], r[1]) for r in model["rows"]]
            else:
                d["key_flags"], d["kid"], d["key"] = 1, np.frombuffer(m.kid, dtype=np.uint8), np.frombuffer(m.key, dtype=np.uint8)
                if family == "cenc":
                    model = CX.demux(m.data, 3, m.n, len(m.runs), 0, room, kid=m.kid, key=m.key)
                else:
                    d["subsample_first"], d["subsample_capacity"] = sub_firsts[i], m.subsamples
                    model = BX.demux(m.data, 3, m.n, len(m.runs), 0, room, kid=m.kid, key=m.key, subsample_capacity=m.subsamples)
                places = [(int(d["dst_offset"]) + off, size) for off, size in model["clear_rows"]]
            assert model["status"] == 0 and model["samples"] == m.n == len(places) and model["runs"] == len(m.runs) == 1
            if gather:
                assert model["gathered"] == b"".join(getattr(m, "clear", None) or [m.data[o:o + k] for o, k in zip(m.offsets, m.sizes)]) and len(model["gathered"]) == clear[i]
                pieces.append((offs[i], bytes(model["gathered"])))
            else:
                assert len(model["gathered"]) == 0
            for k, (place, sample) in enumerate(zip(places, model["samples_rows"])):
                want[1][firsts[i] + k], want[2][firsts[i] + k] = (place[0], place[1], 0), sample
            for k, (place, frame, first_sample, samples, total) in enumerate(model["run_rows"]):
                want[0][run_firsts[i] + k] = (len(src) + place, frame, first_sample, samples, total)
            src += m.data + bytes(-len(m.data) % 4)
        if bad:
            descs["dst_offset"][-1] = dst_bytes
        result = {"mp4f": capi.MP4F_STREAM_RESULT, "cenc": capi.CENC_STREAM_RESULT, "cbcs": capi.CBCS_STREAM_RESULT}[family]
        out = (np.zeros(n, dtype=result), np.zeros(runs, dtype=capi.MP4F_RUN), np.zeros(rows, dtype=capi.ALAC_PACKET), np.zeros(rows, dtype=capi.MP4_SAMPLE))
        head = (_ptr(descs), n, rows, runs) + ((subs,) if family == "cbcs" else ())
        return Case(family, head, [descs], _u8(src), dst_bytes if gather else 0, pieces, sum(len(r) for _, r in pieces), tuple(_ptr(a) for a in out), out, want)

    def _mp4f(self, n, hole, bad, **more):
        return self._frag("mp4f", n, hole, bad, **more)

    def _cenc(self, n, hole, bad, **more):
        return self._frag("cenc", n, hole, bad, **more)

    def _cbcs(self, n, hole, bad, **more):
        return self._frag("cbcs", n, hole, bad, **more)

    def _vorbis(self, n, hole, bad):
        st = VC.stream("mono_64_128")
        ranges = [(0, 4), (4, 5)][:n]
        blob, descs, packets, src, dst_bytes, _ = VF.batch_tables(capi, [st] * n, ranges=ranges)
        pieces = []
        if n:
            descs["dst_offset"][1] += hole
            dst_bytes += hole
            for d, (first, count) in zip(descs, ranges):
                recs, _, pcm = TB.decode_stream(st.model, st.packets[first:first + count])
                assert all(r[0] == TB.OK for r in recs) and 0 < pcm.shape[1] <= int(d["max_samples"])
                pieces.append((int(d["dst_offset"]), VC.pcm_s16be(pcm)))
        else:
            blob, src, dst_bytes = np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), 0
        if bad:
            descs["dst_offset"][-1] = dst_bytes
        out = (np.zeros(n, dtype=capi.VORBIS_STREAM_RESULT), np.zeros(packets.size, dtype=capi.VORBIS_PACKET_RESULT))
        return Case("vorbis", (_ptr(descs), n, _ptr(packets), packets.size, _ptr(blob), blob.size), [descs, packets, blob], src, dst_bytes, pieces,
                    sum(len(r) for _, r in pieces), tuple(_ptr(a) for a in out), out)

    def _ts(self, n, hole, bad):
        rng = TC.Lcg(91)
        job = TC.Job([TC.stream(b"".join(TC.head_packets() + TC.audio_run(rng, n_pes=1 + i, es_bytes=(60, 200))[0])) for i in range(n)])
        if bad:
            job.descs["dst_offset"][-1] = job.dst0.size
        return Case("ts", (_ptr(job.descs), n, job.n_pes), [job.descs], job.src.copy(), job.dst0.size)

    def _adts(self, n, hole, bad):
        rng = TC.Lcg(92)
        job = TC.AdtsJob([TC.adts_stream(b"".join(TC.adts_frame(TC.clean(rng.bytes(20 + 9 * k))) for k in range(2 + i))) for i in range(n)])
        if bad:
            job.descs["src_offset"][-1] = job.src.size
        return Case("adts", (_ptr(job.descs), n, job.n_frames), [job.descs], job.src.copy(), None)

    def _raop_rx(self, n, hole, bad):
        job = XC.Job([XC.stream([XC.A(10 + k) for k in range(2 + i)]) for i in range(n)])
        if bad:
            job.d_grams["src_offset"][-1] = (len(job.src) + 3) & ~3
        return Case("raop_rx", (_ptr(job.d_streams), n, _ptr(job.d_grams), job.d_grams.size), [job.d_streams, job.d_grams], _u8(job.src), None)

    # ---- the calls, by family, returning the library's code
    def check(self, case):
        """The library's own validation of the tables, without a device (raises OhGpuError)."""
        head = case.head[1:] if case.family == "dsd_pcm" else case.head
        lead = self.dsd_key if case.family == "dsd_pcm" else ()
        capi.check(getattr(capi.lib(), f"ohgpu_{case.family}_batch_check")(*lead, *head, *case.sizes()))

    def create(self, case):
        b = C.c_void_p(1)                                           # (a failed create must have nulled it)
        code = getattr(capi.lib(), f"ohgpu_{case.family}_batch_create")(self.ctx.handle, *case.head, *case.sizes(), C.byref(b))
        return code, b

    def run(self, family, batch, d_src, d_dst, stream=None):
        arenas = (d_src,) if family in NO_ARENA else (d_src, d_dst)
        return getattr(capi.lib(), f"ohgpu_{family}_batch_run")(self.ctx.handle, batch, *arenas, stream)

    def process_host(self, case, dst):
        out = () if case.dst_bytes is None else (_ptr(dst), dst.size)
        return getattr(capi.lib(), f"ohgpu_{case.family}_process_host")(self.ctx.handle, *case.head, _ptr(case.src), case.src.size, *out, *case.tail)

    def on_device(self, case):
        """check + create + run + destroy on device arenas: the destination arena afterwards (it starts as DEV_FILL); MPEG-4: its tables."""
        ctx = self.ctx
        self.check(case)
        d_src = ctx.upload(case.src)
        d_dst = ctx.malloc(max(case.dst_bytes or 0, 1))
        ctx.memset(d_dst, DEV_FILL, case.dst_bytes or 0)
        ctx.sync()
        code, b = self.create(case)
        assert code == capi.OK, capi.last_error()
        assert self.run(case.family, b, d_src, d_dst) == capi.OK, capi.last_error()
        ctx.sync()
        if case.family == "mp4":
            got = ctx.mp4_results(b, case.head[1], case.head[2])
        elif case.family in FRAGMENTED:                                # (the arena, then the results and the three tables)
            got = (ctx.download(d_dst, case.dst_bytes),) + getattr(ctx, case.family + "_results")(b, case.head[1], case.head[2], case.head[3])
        elif case.family == "vorbis":
            got = (ctx.download(d_dst, case.dst_bytes),) + ctx.vorbis_results(b, case.head[1], case.head[3])
        else:
            got = ctx.download(d_dst, case.dst_bytes) if case.dst_bytes is not None else None
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        return got


@pytest.fixture(scope="module")
def fx():
    f = Fixtures()
    yield f
    f.close()


@pytest.mark.parametrize("family", FAMILIES + SHELL_ONLY)
def test_failed_create_leaves_nothing_behind(fx, family):
    good = fx.case(family)
    fx.on_device(good)                                              # warm-up: the context's block cache holds this batch's blocks
    allocs = fx.ctx.device_allocations()
    for _ in range(3):
        for bad, code, text in ((("rows", capi.ERR_INVALID, "mp4 desc 1: rows ["), ("file", capi.ERR_BOUNDS, "mp4 desc 1: reads [")) if family == "mp4" else
                                ((True, capi.ERR_BOUNDS, BOUNDS_TEXT[family]),)):
            got, b = fx.create(fx.case(family, bad=bad))
            assert got == code, (got, capi.last_error())
            assert b.value is None
            assert text in capi.last_error(), capi.last_error()
    fx.on_device(good)
    assert fx.ctx.device_allocations() == allocs


@pytest.mark.parametrize("family", FAMILIES)
def test_run_refuses_another_familys_batch(fx, family):
    code, other = fx.create(fx.case("iff" if family == "ogg" else "ogg"))
    assert code == capi.OK
    d = fx.ctx.malloc(4096)
    try:
        for batch in (other, None):
            assert fx.run(family, batch, d, d) == capi.ERR_INVALID
            assert capi.last_error() == f"ohgpu_{family}_batch_run: {NOT_MINE[family]}"
    finally:
        fx.ctx.batch_destroy(other)
        fx.ctx.free(d)


@pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
@pytest.mark.parametrize("family", FAMILIES + SHELL_ONLY)
def test_null_arenas(fx, family, variant):
    """(under kernel variant 1 too: a batch planned onto a plain route needs its arenas no less)"""
    case = fx.case(family)
    fx.ctx.set_kernel_variant(variant)
    try:
        code, b = fx.create(case)
    finally:
        fx.ctx.set_kernel_variant(0)
    assert code == capi.OK, capi.last_error()
    d_src, d_dst = fx.ctx.upload(case.src), fx.ctx.malloc(max(case.dst_bytes or 0, 1))
    try:
        for src, dst in ((None, d_dst), (None, None)) + (() if family in NO_ARENA else ((d_src, None),)):   # (this batch reads source bytes and writes)
            assert fx.run(family, b, src, dst) == capi.ERR_INVALID
            assert capi.last_error() == f"ohgpu_{family}_batch_run: null arena pointer"
    finally:
        fx.ctx.batch_destroy(b)
        fx.ctx.free(d_src)
        fx.ctx.free(d_dst)


@pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
@pytest.mark.parametrize("family", FRAGMENTED)
def test_a_batch_that_gathers_nothing_runs_without_a_destination(fx, family, variant):
    """The fragmented families need the destination arena only when a stream gathers (run_guard's needs_dst): the same files with
    nothing to gather run with a null destination on both routes and leave the model's tables; the source is needed as ever."""
    case = fx.case(family, gather=False)
    fx.check(case)
    fx.ctx.set_kernel_variant(variant)
    try:
        code, b = fx.create(case)
    finally:
        fx.ctx.set_kernel_variant(0)
    assert code == capi.OK, capi.last_error()
    d_src = fx.ctx.upload(case.src)
    try:
        assert fx.run(family, b, None, None) == capi.ERR_INVALID
        assert capi.last_error() == f"ohgpu_{family}_batch_run: null arena pointer"
        assert fx.run(family, b, d_src, None) == capi.OK, capi.last_error()
        res, *tables = getattr(fx.ctx, family + "_results")(b, case.head[1], case.head[2], case.head[3])
        status = res["status"] if family == "mp4f" else res["mp4f"]["status"] if family == "cenc" else res["cenc"]["mp4f"]["status"]
        gathered = res["bytes_gathered"] if family == "mp4f" else res["mp4f"]["bytes_gathered"] if family == "cenc" else res["cenc"]["mp4f"]["bytes_gathered"]
        assert status.tolist() == [0, 0] and gathered.tolist() == [0, 0]
        for got, want in zip(tables, case.want):
            assert got.tobytes() == want.tobytes()
    finally:
        fx.ctx.batch_destroy(b)
        fx.ctx.free(d_src)


@pytest.mark.parametrize("family", FAMILIES + SHELL_ONLY)
def test_empty_batch(fx, family):
    ctx = fx.ctx
    code, b = fx.create(fx.case(family, empty=True))
    assert code == capi.OK, capi.last_error()
    d = ctx.malloc(64)
    try:
        assert ctx.batch_info(b) == ZERO_INFO
        assert fx.run(family, b, d, d) == capi.OK, capi.last_error()
        assert fx.run(family, b, None, None) == capi.OK, capi.last_error()
        ctx.sync()
    finally:
        ctx.batch_destroy(b)
        ctx.free(d)


@pytest.mark.parametrize("hole", [0, HOLE], ids=["adjacent", "hole"])
@pytest.mark.parametrize("family", FAMILIES)
def test_process_host_equals_create_and_run(fx, family, hole):
    case = fx.case(family, hole=hole)
    on_device = fx.on_device(case)
    before = fx.ctx.host_transfer_stats()
    dst = None if case.dst_bytes is None else np.full(case.dst_bytes, HOST_FILL, dtype=np.uint8)
    assert fx.process_host(case, dst) == capi.OK, capi.last_error()
    after = fx.ctx.host_transfer_stats()
    if family == "mp4":                                               # no arena: the tables, with the batch's own fill in the rows of the hole
        for got, dev, want in zip(fx.mp4_results[1:], on_device[1:], fx.mp4_want):
            assert got.tobytes() == dev.tobytes() == want.tobytes()
        assert fx.mp4_results[0].tobytes() == on_device[0].tobytes() and [int(r["status"]) for r in on_device[0]] == [MX.OK, MX.OK]
        assert int(case.head[2]) == sum(int(r["samples"]) for r in on_device[0]) + (HOLE_ROWS if hole else 0)
    elif family == "vorbis":                                          # the PCM lies within 1 LSB of the model's; the two calls write the same bytes
        arena, res, pres = on_device
        assert case.out[0].tobytes() == res.tobytes() and case.out[1].tobytes() == pres.tobytes() and (pres["status"] == 0).all()
        covered = np.zeros(case.dst_bytes, dtype=bool)
        for (off, raw), r in zip(case.pieces, res):
            assert int(r["samples"]) * 2 == len(raw) > 0
            covered[off:off + len(raw)] = True
            mine, model = arena[off:off + len(raw)].view(">i2").astype(np.int32), np.frombuffer(raw, dtype=">i2").astype(np.int32)
            assert int(np.abs(mine - model).max()) <= 1
        assert np.all(arena[~covered] == DEV_FILL) and np.all(dst[~covered] == HOST_FILL) and np.array_equal(dst[covered], arena[covered])
        assert case.pieces[1][0] - case.pieces[0][0] - len(case.pieces[0][1]) >= hole and not covered.all()
    else:
        if family in FRAGMENTED:                                       # the arena, and beside it the tables with the batch's own fill in the rows of the hole
            on_device, results, *tables = on_device
            assert case.out[0].tobytes() == results.tobytes()
            for got, dev, want in zip(case.out[1:], tables, case.want):
                assert got.tobytes() == dev.tobytes() == want.tobytes()
            assert int(case.head[2]) == 3 + 4 + (HOLE_ROWS if hole else 0)
        assert np.array_equal(on_device, case.arena(DEV_FILL))          # create + run: the model's arena, fill and all
        assert np.array_equal(dst, case.arena(HOST_FILL))               # the host-buffer call: the model's bytes, and the host's own everywhere else
        assert len(case.pieces) >= 2 and all(len(raw) > 0 and np.any(np.frombuffer(raw, dtype=np.uint8) != HOST_FILL) for _, raw in case.pieces)
        gap = case.pieces[1][0] - case.pieces[0][0] - len(case.pieces[0][1])
        assert gap >= hole and np.all(dst[case.pieces[0][0] + len(case.pieces[0][1]):case.pieces[1][0]] == HOST_FILL)
    delta = {k: after[k] - before[k] for k in after}
    assert delta == {"calls": 1, "src_calls": 0, "h2d_bytes": case.src.size, "d2h_bytes": case.moved}, (delta, case.moved)
