"""What the RAOP tests share: the committed sessions (tests/golden/raop_textbook.json, made with the system's libcrypto by
tests/golden/make_raop_fixtures.py), fixed-seed keys and payloads, and the batches -- what the C ABI (or the CPU driver) is given and
what the model chain (tests/raop_textbook.py, then tests/alac_textbook.py) says must come of it."""
import json
import os
import struct

import alac_cases as AC
import alac_textbook as T
import raop_textbook as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raop_textbook.json")
PLAINTEXT = 4                    # OHGPU_RAOP_OUT_PLAINTEXT
GUARD, FILL, SCRATCH_FILL = AC.GUARD, AC.FILL, 0x5b

_sessions = None


def sessions():
    """-> [dict(fixture, key, iv, fmtp, cfg, datagrams, payloads, fx)]"""
    global _sessions
    if _sessions is None:
        with open(GOLDEN) as f:
            raw = json.load(f)["sessions"]
        _sessions = []
        for s in raw:
            datagrams = [bytes.fromhex(d) for d in s["datagrams"]]
            _sessions.append(dict(fixture=s["fixture"], key=bytes.fromhex(s["key"]), iv=bytes.fromhex(s["iv"]), fmtp=s["fmtp"], cfg=R.parse_fmtp(s["fmtp"]),
                                  datagrams=datagrams, payloads=[R.parse_datagram(d)["payload"] for d in datagrams], sha256=s["ciphertext_sha256"],
                                  fx=AC.load_fixture(s["fixture"])))
    return _sessions


def session(name):
    return next(s for s in sessions() if s["fixture"] == name)


def rand_bytes(rng, n):
    return bytes(rng.next() & 0xff for _ in range(n))


def stream(key, iv, payloads, form=PLAINTEXT, cfg=None, align=None):
    """one stream of a Job: the key and IV the library is given, the payloads as they arrive, the output form (PLAINTEXT or an
    Apple Lossless form, which takes the stream's configuration), and the source offset mod 16 of all its packets, or of each (None: the Job's)"""
    return dict(key=bytes(key), iv=bytes(iv), payloads=[bytes(p) for p in payloads], form=form, cfg=cfg, align=align)


def session_stream(s, form, key=None):
    return stream(key or s["key"], s["iv"], s["payloads"], form, s["cfg"])


def wrong_key_streams(form_of):
    """-> nine streams that decrypt to bytes no encoder made: every committed session under its key with bit 0x10, then bit 0x01,
    of the first byte flipped, and the last session's packets encrypted under the first session's key and offered under its own.
    form_of(k): the output form of stream k of the nine."""
    out = []
    for s in sessions():
        for bit in (0x10, 0x01):
            wrong = bytes([s["key"][0] ^ bit]) + s["key"][1:]
            out.append(session_stream(s, form_of(len(out)), wrong))
    s, other = sessions()[3], sessions()[0]["key"]
    out.append(stream(s["key"], s["iv"], [R.encrypt_packet(other, s["iv"], p) for p in s["fx"]["packets"]], form_of(len(out)), s["cfg"]))
    return out


def clear_packets(s):
    """what the cipher layer hands the Apple Lossless phases for a stream: its payloads decrypted under the stream's key"""
    return [decrypt_cached(s["key"], s["iv"], p) for p in s["payloads"]]


_clear = {}


def decrypt_cached(key, iv, payload):
    at = (key, iv, payload)
    if at not in _clear:
        _clear[at] = R.decrypt_packet(key, iv, payload)
    return _clear[at]


class Job:
    """streams: [stream(...)].  The payloads are laid into the source arena ROUND ROBIN over the streams (stream 0's first, stream 1's
    first, ..., stream 0's second, ...), packet number q of the arena at the next offset that is `aligns[q % len(aligns)]` mod 16, stray
    bytes in the gaps and none behind the last; the packet table is by stream, as the ABI wants it.  The destination arena: GUARD bytes,
    then a window as long as the source arena which every PLAINTEXT stream writes into at its own first packet's source offset (so the
    window is the source layout moved, decrypted; bytes between packets stay FILL), then the decoding streams' blocks as
    tests/alac_cases.Job lays them.  `want`, `want_packets`, `want_scratch`: the model's; with decode=False the model chain stops behind
    the cipher (want_packets is None and `want` holds the plaintext streams' share only)."""

    def __init__(self, streams, aligns=(0, 4, 8, 12), decode=True):
        self.streams = streams
        src = bytearray()
        where = [[None] * len(s["payloads"]) for s in streams]
        q = 0
        for k in range(max([len(s["payloads"]) for s in streams] + [0])):
            for i, s in enumerate(streams):
                if k >= len(s["payloads"]):
                    continue
                want = aligns[q % len(aligns)] if s["align"] is None else s["align"][k] if isinstance(s["align"], (list, tuple)) else s["align"]
                while len(src) % 16 != want:
                    src.append(0xee)
                where[i][k] = len(src)
                src += s["payloads"][k]
                q += 1
        self.src = bytes(src)
        self.table, at = [], GUARD + (len(src) + 3) // 4 * 4 + GUARD
        for i, s in enumerate(streams):
            s["first_packet"], s["n_packets"] = len(self.table), len(s["payloads"])
            self.table += [(where[i][k], len(p)) for k, p in enumerate(s["payloads"])]
            if s["form"] == PLAINTEXT:
                s["dst_offset"], s["plane_stride"] = GUARD + (where[i][0] if where[i] else 0), 0
                continue
            cfg, span = s["cfg"], len(s["payloads"]) * s["cfg"]["frame_length"]
            if s["form"] == T.PLANAR:
                s["plane_stride"] = span * 4 + GUARD
                size = cfg["channels"] * s["plane_stride"]
            else:
                s["plane_stride"] = 0
                size = (span * cfg["channels"] * (cfg["bit_depth"] // 8) + 3) // 4 * 4 + GUARD
            s["dst_offset"] = at
            at += size
        self.dst0 = bytes([FILL]) * at
        want, scratch = bytearray(self.dst0), bytearray()
        self.want_packets = []
        for i, s in enumerate(streams):
            clear = [decrypt_cached(s["key"], s["iv"], p) for p in s["payloads"]]
            if s["form"] == PLAINTEXT:
                for k, p in enumerate(clear):
                    to = s["dst_offset"] + where[i][k] - where[i][0]
                    want[to:to + len(p)] = p
                self.want_packets += [(T.OK, 0)] * len(clear)
            else:
                for p in clear:
                    scratch += p + bytes([SCRATCH_FILL]) * (-len(p) % 16)
                if decode:
                    self.want_packets += T.render(s["cfg"], clear, s["form"], want, s["dst_offset"], s["plane_stride"], decode_packet=AC.decode_cached)
        if not decode:
            self.want_packets = None
        self.want, self.want_scratch = bytes(want), bytes(scratch)

    def want_streams(self):
        """per stream: (leading OK packets, samples in them, first bad status or 0)"""
        out = []
        for s in self.streams:
            res = self.want_packets[s["first_packet"]:s["first_packet"] + s["n_packets"]]
            ok = 0
            while ok < len(res) and res[ok][0] == T.OK:
                ok += 1
            out.append((ok, sum(n for _, n in res[:ok]), res[ok][0] if ok < len(res) else 0))
        return out

    def driver_blob(self):
        """the job file of tests/cpp/raop_core_driver.cpp"""
        out = [struct.pack("<IIQQ", len(self.streams), len(self.table), len(self.src), len(self.dst0))]
        for s in self.streams:
            out.append(struct.pack("<IIQII", s["first_packet"], s["n_packets"], s["dst_offset"], 1 if s["form"] == PLAINTEXT else 0, 0) + s["key"] + s["iv"])
        out += [struct.pack("<QII", off, size, 0) for off, size in self.table]
        out += [self.src, self.dst0]
        return b"".join(out)


def capi_tables(job):
    """a Job as ohpipeline_amd.capi's (RAOP_STREAM_DESC array, ALAC_PACKET array)"""
    import numpy as np
    from ohpipeline_amd import capi
    descs = np.zeros(len(job.streams), dtype=capi.RAOP_STREAM_DESC)
    for d, s in zip(descs, job.streams):
        if s["cfg"] is not None:
            for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "max_frame_bytes", "avg_bit_rate", "sample_rate"):
                d[k] = s["cfg"][k]
        d["first_packet"], d["n_packets"], d["dst_offset"], d["dst_plane_stride"], d["flags"] = s["first_packet"], s["n_packets"], s["dst_offset"], s["plane_stride"], s["form"]
        d["aes_key"], d["aes_iv"] = list(s["key"]), list(s["iv"])
    packets = np.zeros(len(job.table), dtype=capi.ALAC_PACKET)
    for p, (off, size) in zip(packets, job.table):
        p["src_offset"], p["bytes"] = off, size
    return descs, packets
