"""An independent model of the protected fragmented MPEG-4 layer (ohgpu_cenc_*, include/ohgpu_cenc.h) with the simplest means there
are: the demultiplexer is tests/mp4f_textbook.py's reader, imported and not edited, with the protection boxes read on top of it by
recursion into Python lists; the cipher is tests/raop_textbook.py's encrypt_block -- SubBytes, ShiftRows and MixColumns on a 4 x 4 state,
no T tables --; a counter block is sixteen bytes put together from the IV and an integer; a sample is decrypted a byte at a time.  It
shares no text with csrc/cenc_core.h, and nothing with the muxer pieces of tests/cenc_cases.py.

demux(data, codecs=3, packet_capacity, run_capacity, gather_first_row, dst_capacity, head_only, kid=None, key=None) -> dict: the model of
tests/mp4f_textbook.py's demux (gather always on), and
    entry, scheme, is_protected, iv_size, kid, blocks    the fields ohgpu_cenc_stream_result has behind ohgpu_mp4f_stream_result's
    clear_rows    [(offset from dst_offset, bytes)] per row of `rows`: (0, 0) for a row that is not gathered
    gathered      the CLEAR bytes the decrypt-gather writes

Where this reading differs from the reference's (OpenHome/Media/Codec/Mpeg4.cpp; include/ohgpu_cenc.h carries the same list):
  - the reference reads the version of tenc and senc as (x & 0xF000) >> 24, which is always 0; here the version is the first byte;
  - the reference protects mp4a only; here fLaC and alac are served;
  - the reference holds an IV in Mpeg4ProtectionDetails without checking its size; here the IV is 8 or 16 bytes;
  - the reference hands the cipher to a provider; here the key comes with the call;
  - a library's CTR mode increments all 128 bits of the counter block; here only the low eight bytes count, and they wrap."""
import mp4_textbook as MX
import mp4f_textbook as FX
import raop_textbook as RX

OK, NOT_MP4, TRUNCATED, INVALID, NOT_CODEC, UNSUPPORTED, NOT_FRAGMENTED, NO_KEY = range(8)
RESULT_FIELDS, CONFIG_FIELDS, FLAC_FIELDS = FX.RESULT_FIELDS, FX.CONFIG_FIELDS, FX.FLAC_FIELDS
EXTRA_FIELDS = ("entry", "scheme", "is_protected", "iv_size", "kid", "blocks")
Refuse, u, code = FX.Refuse, FX.u, FX.code


# ---- the keystream
def counter_block(iv, j):
    """counter block j of a sample whose IV is iv (8 or 16 bytes)"""
    low = int.from_bytes(iv[8:16], "big") if len(iv) == 16 else 0
    return bytes(iv[:8]) + ((low + j) % (1 << 64)).to_bytes(8, "big")


_schedules, _blocks = {}, {}


def keystream_block(key, block):
    key, block = bytes(key), bytes(block)
    if (key, block) not in _blocks:
        if key not in _schedules:
            _schedules[key] = RX.key_expansion(key)
        _blocks[(key, block)] = RX.encrypt_block(_schedules[key], block)
    return _blocks[(key, block)]


def keystream(key, iv, n):
    return b"".join(keystream_block(key, counter_block(iv, j)) for j in range((n + 15) // 16))[:n]


def crypt(key, iv, data):
    """one sample: decryption and encryption are the same"""
    return bytes(a ^ b for a, b in zip(data, keystream(key, iv, len(data))))


# ---- the boxes
class Reader(FX.Reader):
    def __init__(self, data, codecs, head_only, kid, key):
        super().__init__(data, codecs, head_only)
        self.kid, self.key = kid, key
        self.ivs = []                   # an IV a sample of a protected track's runs, in order

    def trak(self, box, at, end):
        self.entry_seen = dict(entry=0, scheme=0, is_protected=0, iv_size=0, kid=bytes(16), tenc=0)
        t = super().trak(box, at, end)
        t["prot"] = self.entry_seen
        return t

    def description(self, t, box, pay, end):
        try:
            super().description(t, box, pay, end)
        except Refuse as e:
            if not (e.status == UNSUPPORTED and e.at == pay + 8 and t.get("codec") == code(b"enca")):
                raise
            self.protected_entry(t, pay + 8, end)

    def protected_entry(self, t, entry, end):
        data, prot = self.data, self.entry_seen
        inner = FX.Counter(FX.ENTRY_BOXES)
        _, _, body, entry_end = next(FX.boxes(data, entry, end, inner))
        prot["entry"] = code(b"enca")
        if entry_end - body < 28:
            raise Refuse(INVALID, entry)
        t["entry"] = (u(data, body + 16, 2), u(data, body + 18, 2), u(data, body + 24, 2))
        found = {}
        for kind, child, pay, child_end in FX.boxes(data, body + 28, entry_end, inner):
            if kind == b"sinf" and b"sinf" not in found:
                found[b"sinf"] = child
                for kind2, child2, pay2, end2 in FX.boxes(data, pay, child_end, inner):
                    if kind2 in (b"frma", b"schm") and kind2 not in found:
                        found[kind2] = (child2, pay2, end2)
                    elif kind2 == b"schi" and b"schi" not in found:
                        found[b"schi"] = child2
                        for kind3, child3, pay3, end3 in FX.boxes(data, pay2, end2, inner):
                            if kind3 == b"tenc" and b"tenc" not in found:
                                found[b"tenc"] = (child3, pay3, end3)
            elif kind in (b"dfLa", b"alac") and kind not in found:
                found[kind] = (child, pay, child_end)
        if any(k not in found for k in (b"sinf", b"frma", b"schm", b"tenc")):
            raise Refuse(INVALID, entry)
        for name, least in ((b"frma", 4), (b"schm", 12)):
            if found[name][2] - found[name][1] < least:
                raise Refuse(INVALID, found[name][0])
        prot["scheme"] = u(data, found[b"schm"][1] + 4, 4)
        if prot["scheme"] != code(b"cenc"):
            raise Refuse(UNSUPPORTED, found[b"schm"][0])
        tenc, pay, tenc_end = found[b"tenc"]
        if tenc_end - pay < 24:
            raise Refuse(INVALID, tenc)
        if data[pay] != 0:
            raise Refuse(UNSUPPORTED, tenc)
        if data[pay + 6] > 1:
            raise Refuse(INVALID, tenc)
        if data[pay + 6] == 1 and data[pay + 7] not in (8, 16):
            raise Refuse(UNSUPPORTED, tenc)
        prot.update(is_protected=data[pay + 6], iv_size=data[pay + 7] if data[pay + 6] else 0, kid=data[pay + 8:pay + 24], tenc=tenc)
        t["codec"] = u(data, found[b"frma"][1], 4)
        if t["codec"] == code(b"alac"):
            if b"alac" not in found:
                raise Refuse(UNSUPPORTED, entry)
            child, pay, child_end = found[b"alac"]
            if child_end - pay < 28 or data[pay + 8] != 0:
                raise Refuse(UNSUPPORTED, child)
            cfg, at = {}, pay + 4
            for name, width in zip(CONFIG_FIELDS, (4, 1, 1, 1, 1, 1, 1, 2, 4, 4, 4)):
                cfg[name] = u(data, at, width)
                at += width
            if not (1 <= cfg["channels"] <= 8 and 1 <= cfg["frame_length"] <= 16384 and cfg["bit_depth"] in (16, 20, 24, 32)):
                raise Refuse(UNSUPPORTED, child)
            t.update(config=cfg, parsed=True, limit=cfg["frame_length"] * cfg["channels"] * 5 + 64)
        elif t["codec"] == code(b"fLaC") and self.codecs & FX.CODEC_FLAC:
            if b"dfLa" not in found:
                raise Refuse(UNSUPPORTED, entry)
            self.streaminfo(t, *found[b"dfLa"])

    def streaminfo(self, t, child, pay, end):
        """dfLa, as the clear entry's: version and flags 0, then metadata blocks of which the first is STREAMINFO"""
        data = self.data
        t["parsed"] = True
        if end - pay < 4:
            raise Refuse(INVALID, child)
        if u(data, pay, 4) != 0:
            raise Refuse(UNSUPPORTED, child)
        at, first = pay + 4, True
        while True:
            if end - at < 4 or u(data, at + 1, 3) > end - at - 4:
                raise Refuse(INVALID, child)
            last, kind, length = data[at] >> 7, data[at] & 0x7f, u(data, at + 1, 3)
            if first:
                if kind != 0 or length != 34:
                    raise Refuse(INVALID, child)
                b = data[at + 4:at + 38]
                word = int.from_bytes(b[10:18], "big")
                f = dict(min_blocksize=u(b, 0, 2), max_blocksize=u(b, 2, 2), min_framesize=u(b, 4, 3), max_framesize=u(b, 7, 3), sample_rate=word >> 44,
                         channels=((word >> 41) & 7) + 1, bits=((word >> 36) & 31) + 1, total_samples=word & ((1 << 36) - 1), md5=bytes(b[18:34]))
                if f["bits"] not in (8, 16, 24):
                    raise Refuse(UNSUPPORTED, child)
                t.update(flac=f, limit=f["max_blocksize"] * f["channels"] * (f["bits"] // 8 + 1) + 64)
                first = False
            at += 4 + length
            if last or at == end:
                return

    def movie(self, box, at, end):
        super().movie(box, at, end)
        prot = self.track["prot"]
        if prot["is_protected"] and not self.head_only and (self.key is None or bytes(self.kid) != bytes(prot["kid"])):
            raise Refuse(NO_KEY, prot["tenc"])

    def fragment(self, moof, at, end):
        """the sibling's reading of a moof (its header, its runs), and at the end of each traf of the taken track what its other boxes say"""
        data, trafs = self.data, 0
        for kind, traf, pay, traf_end in FX.boxes(data, at, end, self.counter):
            if kind != b"traf":
                continue
            trafs += 1
            head, first_run, time, senc, seig = None, True, None, None, None
            runs_before, samples_before = len(self.runs), self.samples
            for kind2, child, pay2, end2 in FX.boxes(data, pay, traf_end, self.counter):
                if kind2 == b"tfhd" and head is None:
                    head = self.fragment_header(child, pay2, end2, moof, trafs == 1)
                    continue
                if kind2 not in (b"tfdt", b"trun"):
                    if kind2 == b"senc" and senc is None:
                        senc = (child, pay2, end2)
                    if kind2 in (b"sbgp", b"sgpd") and seig is None and end2 - pay2 >= 8 and data[pay2 + 4:pay2 + 8] == b"seig":
                        seig = child
                    continue
                if head is None:
                    raise Refuse(INVALID, child)
                if head is False:
                    continue
                if kind2 == b"tfdt":
                    if first_run and time is None:
                        v = FX.versioned(data, child, pay2, end2, 8, 12)
                        time = u(data, pay2 + 4, 8 if v else 4)
                    continue
                run = self.run(child, pay2, end2, head)
                if run is None:
                    continue
                run["place"] = head["base"] + run["offset"] if run["offset"] is not None else head["base"] if first_run else None
                run["time"] = time if first_run else None
                first_run = False
                self.runs.append(run)
            if head is None:
                raise Refuse(INVALID, traf)
            if head is not False:
                self.judge(traf, senc, seig, self.samples - samples_before)

    def judge(self, traf, senc, seig, samples):
        data, prot = self.data, self.track["prot"]
        if seig is not None:
            raise Refuse(UNSUPPORTED, seig)
        if not prot["is_protected"]:
            return
        if senc is None:
            if samples:
                raise Refuse(UNSUPPORTED, traf)
            return
        box, pay, end = senc
        if end - pay < 8:
            raise Refuse(INVALID, box)
        if data[pay] != 0 or data[pay + 3] & 3:
            raise Refuse(UNSUPPORTED, box)
        count, size = u(data, pay + 4, 4), prot["iv_size"]
        if count * size > end - pay - 8 or count != samples:
            raise Refuse(INVALID, box)
        self.ivs += [data[pay + 8 + k * size:pay + 8 + (k + 1) * size] for k in range(count)]


def demux(data, codecs=3, packet_capacity=1 << 20, run_capacity=1 << 20, gather_first_row=0, dst_capacity=0, head_only=False, kid=None, key=None):
    data = bytes(data)
    r = Reader(data, codecs, head_only, kid, key)
    # the sibling's demux() over this reader: its Reader is looked up when it runs
    sibling = FX.Reader
    FX.Reader = lambda d, c, h: r
    try:
        out = FX.demux(data, codecs, packet_capacity, run_capacity, True, gather_first_row, dst_capacity, head_only)
    finally:
        FX.Reader = sibling
    out.update(entry=0, scheme=0, is_protected=0, iv_size=0, kid=bytes(16), blocks=0, clear_rows=[(0, 0)] * len(out["rows"]))
    if out["status"] == NO_KEY:                       # what moov gave is kept: the sibling's reading of the same bytes up to moov's end
        head = demux(data, codecs, head_only=True)
        out.update({k: head[k] for k in ("codec", "track_id", "timescale", "duration", "entry_rate", "entry_channels", "entry_bits", "moov_offset", "config", "flac")})
    if out["status"] not in (OK, NO_KEY):
        return out
    prot = r.track["prot"]
    out.update(entry=prot["entry"] or r.track["codec"], scheme=prot["scheme"], is_protected=prot["is_protected"], iv_size=prot["iv_size"], kid=bytes(prot["kid"]))
    if not out["bytes_gathered"]:
        return out
    clear, at = [], 0
    for row in range(gather_first_row, out["samples_available"]):
        place, size = out["rows"][row]
        sample = data[place:place + size]
        if prot["is_protected"]:
            sample = crypt(key, r.ivs[row], sample)
            out["blocks"] += (size + 15) // 16
        out["clear_rows"][row] = (at, size)
        clear.append(sample)
        at += size
    out["gathered"] = b"".join(clear)
    assert len(out["gathered"]) == out["bytes_gathered"]
    return out
